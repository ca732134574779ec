"""CPU tests (-m "not gpu"): the C-ABI library loads and exports every symbol include/gdrn_hip.h declares, host-side
logic (config gate, state-dict schema, synthetic inputs, Ranger scalars), and the product path refuses to run
without a GPU (no silent CPU fallback)."""
import os
import re

import numpy as np
import pytest
import torch

from gdrnet_amd import cabi, synth
from gdrnet_amd.cfg import lm13_cfg, lmo_cfg, ycbv_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|long long)\s+(gdrn_[a-z0-9_]+)\s*\(", txt)))


def test_library_loads_and_exports_every_declared_symbol():
    if not os.path.exists(cabi.LIB_PATH):
        from gdrnet_amd import build

        build.build(verbose=False)
    lib = cabi.load()
    declared = _header_symbols()
    assert len(declared) >= 35
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/gdrn_hip.h but not exported"
    assert sorted(cabi.EXPORTS) == declared, set(cabi.EXPORTS) ^ set(declared)
    assert lib.gdrn_version() == 5  # host-only call (no device needed)


def test_struct_layouts_match_the_header():
    """field order of the ctypes mirrors == field order of the C structs."""
    txt = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for cname, cls in (("gdrn_conv_params", cabi.ConvParams), ("gdrn_wgrad_params", cabi.WgradParams), ("gdrn_pose_params", cabi.PoseParams),
                       ("gdrn_pack_task", cabi.PackTask), ("gdrn_ranger_task", cabi.RangerTask), ("gdrn_wreduce_task", cabi.WreduceTask),
                       ("gdrn_roi_task", cabi.RoiTask), ("gdrn_s2_params", cabi.S2Params), ("gdrn_s2d_params", cabi.S2dParams)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            names = re.sub(r"^(const\s+)?(void|float|int|double|long long|unsigned char)\s*\*?", "", decl)
            fields += [n.strip().lstrip("*").strip() for n in names.split(",")]
        assert fields == [f[0] for f in cls._fields_], cname


def test_state_dict_schema_and_param_count():
    from gdrnet_amd import GDRN

    model, opt = GDRN.build_model_optimizer(lm13_cfg(device="cpu"))
    sd = model.state_dict()
    schema = synth.param_schema()
    assert list(sd.keys()) == list(schema.keys())
    for k, (shape, _) in schema.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    assert sum(p.numel() for p in model.parameters()) == 35054094 and len(list(model.parameters())) == 148
    assert len(opt.param_groups) == 3 and all(abs(g["lr"] - 1e-4) < 1e-12 for g in opt.param_groups)
    assert model.load_state_dict(synth.make_state_dict(0)).missing_keys == []
    # reference init: N(0, 0.001^2) convs, fc_r / fc_t 0.01, BN / GN weight 1
    m2, _ = GDRN.build_model_optimizer(lmo_cfg(device="cpu"))
    assert 5e-4 < float(m2.backbone.layer1[0].conv1.weight.std()) < 2e-3
    assert 5e-3 < float(m2.pnp_net.fc_r.weight.std()) < 2e-2
    assert float(m2.rot_head_net.features[1].weight.min()) == 1.0
    assert GDRN.get_xyz_mask_region_out_dim(m2.cfg) == (3, 1, 65)


def test_no_cpu_fallback_and_scope_gate():
    from gdrnet_amd import GDRN

    model, _ = GDRN.build_model_optimizer(lm13_cfg(device="cpu"))
    b = synth.make_batch(2, seed=1)
    with pytest.raises(cabi.GdrnHipError):
        model(b["roi_img"], **synth.model_kwargs(b, do_loss=False))
    with pytest.raises(RuntimeError):
        model.backbone(b["roi_img"])  # sub-modules are parameter containers
    for mutate in (lambda c: c.MODEL.CDPN.PNP_NET.__setitem__("ROT_TYPE", "ego_quat"),
                   lambda c: c.MODEL.CDPN.ROT_HEAD.__setitem__("XYZ_LOSS_TYPE", "CE_coor"),
                   lambda c: c.MODEL.CDPN.BACKBONE.__setitem__("NUM_LAYERS", 50),
                   lambda c: c.MODEL.CDPN.TRANS_HEAD.__setitem__("ENABLED", True)):
        cfg = ycbv_cfg(device="cpu")
        mutate(cfg)
        with pytest.raises(NotImplementedError):
            GDRN.build_model_optimizer(cfg)


def test_synthetic_inputs_are_deterministic_and_shaped_like_batch_data():
    a, b = synth.make_batch(3, seed=5, as_torch=False), synth.make_batch(3, seed=5, as_torch=False)
    for k in a:
        if k != "sym_info":
            assert np.array_equal(a[k], b[k]), k
    assert a["roi_img"].shape == (3, 3, 256, 256) and a["roi_img"].dtype == np.float32
    assert a["roi_coord_2d"].shape == (3, 2, 64, 64) and a["roi_region"].dtype == np.int64
    assert a["roi_points"].shape == (3, 3000, 3) and a["roi_mask_visib"].shape == (3, 64, 64)
    R = a["ego_rot"].astype(np.float64)
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-6)
    assert not np.array_equal(a["roi_img"], synth.make_batch(3, seed=6, as_torch=False)["roi_img"])
    u = synth.hash_uniform(1, "x", (100000,))
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 5e-3
    assert abs(synth.hash_normal(1, "y", (100000,)).std() - 1.0) < 1e-2


def test_ranger_rectification_scalars_match_reference_golden(golden_dir):
    """radam_step_size reproduces the host arithmetic of lib/torch_utils/solver/ranger.py:154-186; a pure-numpy Ranger
    built on it replays the reference's 7 golden steps (tests/golden/g6_ranger.npz)."""
    from gdrnet_amd.ranger import radam_step_size

    g = np.load(os.path.join(golden_dir, "g6_ranger.npz"))
    ps = [synth.hash_normal(31, f"p{i}", s).astype(np.float32) for i, s in enumerate(((8, 4, 3, 3), (16, 8), (16,)))]
    m = [np.zeros_like(p) for p in ps]
    v = [np.zeros_like(p) for p in ps]
    slow = [p.copy() for p in ps]
    lr, b1, b2, eps = 1e-2, 0.95, 0.999, 1e-5
    for step in range(1, 8):
        n_sma, ss = radam_step_size(step, b1, b2, 5)
        for i, p in enumerate(ps):
            gr = synth.hash_normal(32 + step - 1, f"g{i}", p.shape).astype(np.float32)
            if gr.ndim > 1:
                gr = gr - gr.reshape(gr.shape[0], -1).mean(1).reshape((-1,) + (1,) * (gr.ndim - 1))
            v[i] = v[i] * np.float32(b2) + np.float32(1 - b2) * gr * gr
            m[i] = m[i] * np.float32(b1) + np.float32(1 - b1) * gr
            if n_sma > 5:
                p -= np.float32(ss * lr) * m[i] / (np.sqrt(v[i]) + np.float32(eps))
            else:
                p -= np.float32(ss * lr) * m[i]
            if step % 6 == 0:
                slow[i] += np.float32(0.5) * (p - slow[i])
                p[...] = slow[i]
            np.testing.assert_allclose(p, g[f"step{step - 1}/p{i}"], rtol=2e-5, atol=2e-7)


def test_postproc_has_no_cpu_fallback():
    """the on-device inference post-processing refuses CPU tensors instead of silently computing on the host."""
    import torch

    from gdrnet_amd import cabi, postproc

    cfg = lm13_cfg(device="cpu")
    m = torch.rand(2, 1, 64, 64)
    with pytest.raises(cabi.GdrnHipError):
        postproc.get_out_mask(cfg, m)
    with pytest.raises(cabi.GdrnHipError):
        postproc.get_out_coor(cfg, m, m, m)


def test_workspace_bytes_query_matches_the_per_op_rules():
    """gdrn_workspace_bytes (host-only, no device needed): the sizes a non-Python host allocates == the rules the engine uses."""
    import ctypes as C

    lib = cabi.load()
    cp = cabi.ConvParams()
    cp.Hi = cp.Wi = cp.Ho = cp.Wo = 64
    cp.Cin = cp.Cout = cp.x_cs = cp.y_cs = 256
    cp.KH = cp.KW = 3
    cp.stride = cp.pad = 1
    cp.M, cp.dtype, cp.w_rows = 64 * 4096, cabi.BF16, 256
    rows = lib.gdrn_conv3x3_stats_rows(C.byref(cp))
    assert rows == 64 * 4096 // 128
    assert lib.gdrn_workspace_bytes(1, C.byref(cp)) == rows * 2 * 256 * 4
    assert lib.gdrn_workspace_bytes(0, C.byref(cp)) == lib.gdrn_conv_stats_rows(C.byref(cp)) * 2 * 256 * 4
    wp = cabi.WgradParams()
    wp.Hi = wp.Wi = wp.Ho = wp.Wo = 16
    wp.Cin = wp.Cout = wp.x_cs = wp.dy_cs = 256
    wp.KH = wp.KW = 3
    wp.stride = wp.pad = 1
    wp.M, wp.dtype, wp.splits = 64 * 256, cabi.BF16, 4
    assert lib.gdrn_workspace_bytes(2, C.byref(wp)) == 4 * 256 * 256 * 9 * 4
    n = C.c_int(64)
    assert lib.gdrn_workspace_bytes(3, C.byref(n)) == lib.gdrn_stem_wgrad_parts(64) * 64 * 224 * 4
    assert lib.gdrn_workspace_bytes(4, C.byref(n)) == lib.gdrn_stem_stats_rows(64) * 2 * 64 * 4
    mn = (C.c_int * 2)(64, 1024)
    assert lib.gdrn_workspace_bytes(5, mn) == (16 * 64 * 1024 + 64) * 4
    a = (C.c_longlong * 3)(64 * 4096, 256, cabi.BF16)
    assert lib.gdrn_workspace_bytes(6, a) == lib.gdrn_bn_bwd_reduce_rows(64 * 4096, 256, cabi.BF16) * 2 * 256 * 4
    assert lib.gdrn_workspace_bytes(99, a) == -1 and lib.gdrn_workspace_bytes(0, None) == -1


def test_c_client_compiles_links_and_runs(tmp_path):
    """include/gdrn_hip.h is a C header whose documented names (GDRN_ERR_*, GDRN_DT_*) are the ones it defines: a pure-C client is
    compiled with gcc, linked against libgdrn_hip.so and run (host-only queries: no GPU needed)."""
    import shutil
    import subprocess

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lib = cabi.lib_path()
    if not os.path.exists(lib):
        pytest.skip("library not built")
    exe = str(tmp_path / "c_client")
    libdir = os.path.dirname(lib)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_client.c"),
                           "-L", libdir, "-lgdrn_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "gdrn C client ok" in out.stdout


def test_pretrained_backbone_is_resolved_from_the_hub_cache_or_refused(tmp_path, monkeypatch):
    """configs/_base_/gdrn_base.py:21 names "torchvision://resnet34": found in $TORCH_HOME/hub/checkpoints it is loaded (strict=False, as
    mmcv's load_checkpoint at GDRN.py:721); absent, the build refuses instead of silently training from the random init."""
    from gdrnet_amd import GDRN

    cfg = lm13_cfg(device="cpu")
    cfg.MODEL.CDPN.BACKBONE.PRETRAINED = "torchvision://resnet34"
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="hub"):
        GDRN.build_model_optimizer(cfg)
    ref, _ = GDRN.build_model_optimizer(lm13_cfg(device="cpu"))
    sd = {k: torch.full_like(v, 0.25) for k, v in ref.backbone.state_dict().items() if k.startswith("layer1.0.conv1")}
    os.makedirs(tmp_path / "hub" / "checkpoints")
    torch.save(sd, tmp_path / "hub" / "checkpoints" / "resnet34-b627a593.pth")
    cfg2 = lm13_cfg(device="cpu")
    cfg2.MODEL.CDPN.BACKBONE.PRETRAINED = "torchvision://resnet34"
    m, _ = GDRN.build_model_optimizer(cfg2)
    assert float(m.backbone.layer1[0].conv1.weight.mean()) == 0.25
    # mmcv's zoo names are NOT torchvision's files (different, caffe-style weights under the same model name): refused, not mapped
    cfg3 = lm13_cfg(device="cpu")
    cfg3.MODEL.CDPN.BACKBONE.PRETRAINED = "open-mmlab://resnet34"
    with pytest.raises(FileNotFoundError):
        GDRN.build_model_optimizer(cfg3)
    # two candidate files: ambiguous, refused
    torch.save(sd, tmp_path / "hub" / "checkpoints" / "resnet34-333f7ec4.pth")
    cfg4 = lm13_cfg(device="cpu")   # (a built config is consumed: build_model_optimizer pops PNP_HEAD_CFG.type, as GDRN.py:658-659)
    cfg4.MODEL.CDPN.BACKBONE.PRETRAINED = "torchvision://resnet34"
    with pytest.raises(FileNotFoundError):
        GDRN.build_model_optimizer(cfg4)


def test_fp16_library_build_exports_the_same_abi():
    """libgdrn_hip_f16.so = the same sources with IEEE half as the 16-bit format (csrc/common.h): same entry points, it reports GDRN_DT_F16
    as its 16-bit dtype code and the loader refuses a library of the wrong kind."""
    if not os.path.exists(cabi.LIB_PATH_F16):
        from gdrnet_amd import build

        build.build(verbose=False)
    lib = cabi.load(cabi.F16)
    for name in _header_symbols():
        assert hasattr(lib, name), name
    assert lib.gdrn_half_format() == cabi.F16 == 2 and cabi.load(cabi.BF16).gdrn_half_format() == cabi.BF16 == 1
    assert lib is not cabi.load(cabi.BF16) and cabi.load(cabi.F32) is cabi.load(cabi.BF16)


def _dry_engine(dtype="bf16"):
    from gdrnet_amd import GDRN
    from gdrnet_amd.engine import Engine

    model, _ = GDRN.build_model_optimizer(lm13_cfg(device="cpu"))
    return Engine(dict(model.named_parameters()), dict(model.named_buffers()), dtype=dtype, dry=True)


def test_engine_switches_are_validated_and_the_library_reads_no_environment(monkeypatch):
    """r5: 18 documented switches, every one of them read by the Python host with a checked value set; the C-ABI library
    itself calls getenv nowhere -- its choices are functions of the params (host-only queries below, no GPU)."""
    import glob

    csrc = os.path.join(ROOT, "gdr-net_amd", "csrc")
    for f in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")):
        assert "getenv" not in open(f).read(), f
    for var, bad in (("GDRN_WGRAD_STREAM", "2"), ("GDRN_HALO_F32", "yes"), ("GDRN_V3", "1"), ("GDRN_BUCKETS", "3")):
        monkeypatch.setenv(var, bad)
        with pytest.raises(ValueError, match=var):
            _dry_engine()
        monkeypatch.delenv(var)
    # defaults and the documented alternatives
    e = _dry_engine()
    assert (e.wgrad_stream, e.wgrad_force_lds, e.wgrad_blocks) == (True, False, 768) and (e.v3_policy, e.v3_min_wg) == (0, 0)
    assert e.loss_scale == 1.0 and not e.loss_scale_dynamic
    monkeypatch.setenv("GDRN_WGRAD_STREAM", "serial")
    e = _dry_engine()
    assert (e.wgrad_stream, e.wgrad_force_lds, e.wgrad_blocks) == (False, True, 768)   # one stream, the two-stream step's launch configuration
    monkeypatch.setenv("GDRN_WGRAD_STREAM", "0")
    assert _dry_engine().wgrad_blocks == 1536
    monkeypatch.delenv("GDRN_WGRAD_STREAM")
    monkeypatch.setenv("GDRN_V3", "2")
    e = _dry_engine()
    assert (e.v3_policy, e.v3_min_wg) == (2, 1)
    monkeypatch.delenv("GDRN_V3")
    # fp16: "<initial scale>[:<growth interval> | :static]"
    for spec, want in ((None, (1024.0, True, 2000)), ("512", (512.0, True, 2000)), ("256:50", (256.0, True, 50)), ("1024:static", (1024.0, False, 0))):
        if spec is None:
            monkeypatch.delenv("GDRN_LOSS_SCALE", raising=False)
        else:
            monkeypatch.setenv("GDRN_LOSS_SCALE", spec)
        e = _dry_engine("fp16")
        assert (e.loss_scale, e.loss_scale_dynamic, e.loss_scale_growth) == want, spec
    monkeypatch.delenv("GDRN_LOSS_SCALE", raising=False)
    # fp32 parity mode: the halo tile in plans of >= 32 RoIs by default, both operand layouts kept
    e = _dry_engine("fp32")
    assert e.use_halo and e.halo_min_b == 32
    k64 = {getattr(op, "meta", {}).get("kernel") for op in e.plan(64, True, True).fwd}
    k4 = {getattr(op, "meta", {}).get("kernel") for op in e.plan(4, True, True).fwd}
    assert any(k and k.startswith("conv3x3_halo_kernel<f32") for k in k64) and not any(k and k.startswith("conv3x3_halo_kernel") for k in k4)


def test_switch_table_is_the_documented_one_and_the_only_reader_of_the_environment(monkeypatch):
    """gdrnet_amd.switches: its table names exactly the variables of INTEGRATION.md section 3 (one row each, the heading counts them), no other
    module of the package looks a GDRN_* name up in the environment, and every switch read by the engine's constructor refuses an undocumented
    value with a ValueError that names the variable."""
    import glob

    from gdrnet_amd import switches
    from gdrnet_amd.engine import Engine

    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 3. Environment switches"):doc.index("## 4. ")]
    rows = [[c.strip() for c in re.split(r"(?<!\\)\|", ln)[1:-1]] for ln in sec.splitlines() if ln.startswith("| `GDRN_")]   # variable | default | read at | effect
    names = [re.match(r"`(GDRN_[A-Z0-9_]+)`", r[0]).group(1) for r in rows]
    assert sorted(names) == sorted(switches.TABLE) and len(names) == len(set(names))
    assert int(re.match(r"## 3\. Environment switches \((\d+);", sec).group(1)) == len(names)
    assert [r[2] for r in rows] == [switches.TABLE[n].read_at for n in names]
    near = re.compile(r"\benviron\b[^\n]*GDRN_[A-Z0-9_]+|GDRN_[A-Z0-9_]+[^\n]*\benviron\b")   # on one line with os.environ
    hits = [os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "gdr-net_amd", "*.py")) if near.search(open(f).read())]
    assert set(hits) <= {"switches.py"}, hits
    bad = {"GDRN_WGRAD_STREAM": "2", "GDRN_HALO_F32": "yes", "GDRN_V3": "1", "GDRN_BUCKETS": "3", "GDRN_GEMM_BNB": "yes", "GDRN_FUSE_XF": "2",
           "GDRN_HALO_WAVES": "6", "GDRN_FUSE_UP": "on", "GDRN_FC_TAIL": "", "GDRN_MAX_PLANS": "0", "GDRN_LOSS_SCALE": "1024:often"}
    assert set(bad) == {s.name for s in switches.TABLE.values() if s.read_at == switches.ENGINE}
    params, buffers = {"backbone.conv1.weight": torch.zeros(64, 3, 7, 7)}, {}   # (the constructor reads its switches before it looks at a layer)
    for var, value in bad.items():
        monkeypatch.setenv(var, value)
        with pytest.raises(ValueError, match=var):
            Engine(params, buffers, dtype="bf16", dry=True)
        monkeypatch.delenv(var)
    for var, value in (("GDRN_EARLY_OPT", "yes"), ("GDRN_GRAPH", "2"), ("GDRN_DP_CHECK_STEPS", "-1"), ("GDRN_HIP_DTYPE", "fp8")):
        monkeypatch.setenv(var, value)
        with pytest.raises(ValueError, match=var):
            switches.read(var)
        monkeypatch.delenv(var)
    assert switches.read("GDRN_EARLY_OPT") is True and switches.read("GDRN_GRAPH") is False and switches.read("GDRN_DP_CHECK_STEPS") == 2


def test_update_schedule_truth_table(monkeypatch):
    """GDRN._update_schedule, the decision of train_step's three tails, row by row as train_step's expression had it before the split: the
    per-bucket update needs an optimizer that has it, two streams, GDRN_EARLY_OPT, and either nothing attached or the model's own deferred-scale
    reducer (on the GPU, or inactive); a dynamic loss-scale state overrides everything."""
    from types import SimpleNamespace as NS

    from gdrnet_amd.GDRN import _update_schedule

    monkeypatch.delenv("GDRN_EARLY_OPT", raising=False)
    ranger, sgd = NS(step_buckets_begin=None, step=None), NS(step=None)
    two, one = NS(wgrad_stream=True), NS(wgrad_stream=False)
    hook = lambda b: None

    def red(**kw):
        return NS(**dict(dict(on_bucket=hook, defer_scale=True, cuda=True, active=True), **kw))

    assert _update_schedule(ranger, None, None, two, None) == "per_bucket"
    assert _update_schedule(ranger, None, None, one, None) == "whole"              # GDRN_WGRAD_STREAM=0 / serial
    assert _update_schedule(None, None, None, two, None) == "whole"
    assert _update_schedule(sgd, None, None, two, None) == "whole"                 # no step_buckets_begin
    assert _update_schedule(ranger, red(), hook, two, None) == "per_bucket"        # the model's reducer, on the GPU
    assert _update_schedule(ranger, red(defer_scale=False), hook, two, None) == "whole"
    assert _update_schedule(ranger, red(), lambda b: None, two, None) == "whole"   # somebody else's hook
    assert _update_schedule(ranger, red(cuda=False), hook, two, None) == "whole"   # active reducer off the GPU
    assert _update_schedule(ranger, red(cuda=False, active=False), hook, two, None) == "per_bucket"
    assert _update_schedule(ranger, None, hook, two, None) == "whole"              # on_bucket set without a reducer
    dyn = NS(ptr=0)
    for args in ((ranger, None, None, two), (None, None, None, one), (sgd, red(cuda=False), hook, one), (ranger, None, hook, two)):
        assert _update_schedule(*args, dyn) == "guarded"
    monkeypatch.setenv("GDRN_EARLY_OPT", "0")
    assert _update_schedule(ranger, None, None, two, None) == "whole" and _update_schedule(ranger, red(), hook, two, None) == "whole"
    assert _update_schedule(ranger, None, None, two, dyn) == "guarded"


def test_kernel_form_and_layout_queries_are_functions_of_the_params():
    """gdrn_conv3x3_halo_waves / gdrn_conv3x3_wfrag (host-only): the eight-wave form for grids of <= 256 workgroups of the 128-channel tile unless
    halo_waves forbids it; w_frag of the query is the caller's policy (0 library, 1 never the second-generation kernel, 2 wherever covered)."""
    import ctypes as C

    lib = cabi.load()

    def cp(C_, Hh, B, **kw):
        p = cabi.ConvParams()
        p.Hi = p.Wi = p.Ho = p.Wo = Hh
        p.Cin = p.x_cs = p.Cout = p.y_cs = C_
        p.KH = p.KW = 3
        p.stride, p.pad = 1, 1
        p.M, p.w_rows, p.dtype = B * Hh * Hh, C_, cabi.BF16
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert lib.gdrn_conv3x3_halo_waves(C.byref(cp(256, 16, 64))) == 8          # 256 workgroups: one per CU -> eight waves
    assert lib.gdrn_conv3x3_halo_waves(C.byref(cp(512, 8, 64))) == 8
    assert lib.gdrn_conv3x3_halo_waves(C.byref(cp(128, 32, 64))) == 4          # 512 workgroups
    assert lib.gdrn_conv3x3_halo_waves(C.byref(cp(256, 16, 64, halo_waves=4))) == 4
    assert lib.gdrn_conv3x3_halo_waves(C.byref(cp(128, 32, 64, halo_waves=8))) == 8
    assert lib.gdrn_conv3x3_halo_waves(C.byref(cp(64, 64, 64))) == 4           # the 64-channel tile has no eight-wave form
    assert lib.gdrn_conv3x3_halo(C.byref(cp(256, 16, 64, halo_waves=5)), None) == -1   # GDRN_ERR_ARG before anything is launched (null x / w / y)
    # layout query: plain launches prefer the first kernel, transformed 256-channel ones on large grids the second-generation kernel
    assert lib.gdrn_conv3x3_wfrag(C.byref(cp(256, 64, 64))) == 1
    assert lib.gdrn_conv3x3_wfrag(C.byref(cp(256, 64, 64, xf_mode=1))) == 2
    assert lib.gdrn_conv3x3_wfrag(C.byref(cp(256, 64, 64, xf_mode=1, w_frag=1))) == 1     # policy: never
    assert lib.gdrn_conv3x3_wfrag(C.byref(cp(256, 64, 64, w_frag=2))) == 2                # policy: wherever covered
    assert lib.gdrn_conv3x3_wfrag(C.byref(cp(256, 64, 64, w_frag=7))) == -1
    # the 256-channel tile of the second-generation kernel only on grids of >= 256 workgroups unless v3_min_wg lowers the threshold
    th, tw, bn = C.c_int(0), C.c_int(0), C.c_int(0)
    small = cp(256, 16, 4, xf_mode=1, w_frag=2)
    lib.gdrn_conv3x3_tile(C.byref(small), C.byref(th), C.byref(tw), C.byref(bn))
    assert (th.value, tw.value, bn.value) == (8, 16, 128)
    small.v3_min_wg = 1
    lib.gdrn_conv3x3_tile(C.byref(small), C.byref(th), C.byref(tw), C.byref(bn))
    assert (th.value, tw.value, bn.value) == (16, 16, 256)
    name = C.create_string_buffer(32)
    assert lib.gdrn_last_hip_error(name, 32) == 0   # no launch of this thread has failed


def test_norm_entry_points_refuse_shapes_their_kernels_cannot_hold():
    """Host-side argument checks of csrc/norm.hip, before anything is launched (every pointer is a valid HOST buffer: a call that got past its
    checks would return -3, launch failure, on a box without a device).  bn_apply_kernel stages scale / shift in kst[2][512]: gdrn_bn_apply
    refuses C > 512 (GDRN_ERR_ARG, like gdrn_bn_bwd_apply / gdrn_bn_bwd_reduce) -- C = 1024 in either type and C = 2048 in the 16-bit type pass
    its C % 8 and C / V <= 256 checks.  gdrn_maxpool_bwd with rows keeps a thread on one channel vector over its grid-stride trips only for
    C / V dividing 64; gdrn_upsample2x_bwd_bnsums needs C / V to divide 256."""
    import torch

    for kind in (cabi.BF16, cabi.F16):
        lib = cabi.load(kind)
        buf = torch.zeros(4096)
        p = buf.data_ptr()
        for C_, dt in ((1024, cabi.F32), (1024, kind), (2048, kind)):
            assert lib.gdrn_bn_apply(p, p, p, None, p, 1, C_, 1, dt, None) == -1, (C_, dt)
            assert lib.gdrn_bn_apply(p, p, p, p, p, 1, C_, 0, dt, None) == -1, (C_, dt)
        assert lib.gdrn_bn_apply(p, p, p, None, p, 1, 2048, 1, cabi.F32, None) == -1
        assert lib.gdrn_bn_bwd_apply(p, None, p, p, p, p, None, None, 1, 1024, p, None, kind, None) == -1     # the siblings' bound
        assert lib.gdrn_bn_bwd_reduce(p, None, p, p, p, None, None, 1, 1024, p, kind, None) == -1
        # rows: fp32 C = 512 is 128 channel vectors (> 64); without rows the same shape is accepted by the checks (and not run here)
        assert lib.gdrn_maxpool_bwd(p, p, p, p, p, p, 1, 2, 2, 512, p, p, p, cabi.F32, None) == -2
        assert lib.gdrn_maxpool_bwd(p, p, p, p, p, p, 1, 2, 2, 512, None, None, p, cabi.F32, None) == -1      # rows without mean / invstd
        for dt in (cabi.F32, kind):   # C / V = 6 or 3: does not divide 256
            assert lib.gdrn_upsample2x_bwd_bnsums(p, p, p, p, p, p, p, 1, 2, 2, 24, p, dt, None) == -2, dt
            assert lib.gdrn_bn_bwd_reduce_rows(4, 24, dt) == -2


def test_build_is_stamped_with_the_source_hash(tmp_path, monkeypatch):
    """VERDICT r4 'weak' 10: build() decides by CONTENT -- a library whose stamp does not match the sources (or has none) is rebuilt, whatever the
    file times say."""
    from gdrnet_amd import build as B

    assert os.path.exists(B.STAMP) and open(B.STAMP).read().strip() == B.source_hash() and not B.needs_build()
    stamp = tmp_path / "source_hash.txt"
    monkeypatch.setattr(B, "STAMP", str(stamp))
    assert B.needs_build()                          # no stamp
    stamp.write_text("0123456789abcdef\n")
    assert B.needs_build()                          # a stamp of other sources, however new the file is
    stamp.write_text(B.source_hash() + "\n")
    assert not B.needs_build()


def test_plans_route_the_stem_and_the_head_output_conv_to_their_own_kernels():
    """r5 wiring on dry plans (launch lists only): inference runs the stem as one kernel and the 1x1 output conv + head tail as one kernel and the
    small-map convs in the eight-wave form; the training step runs the output conv + tail + map losses as one kernel, its data gradient on
    head_out_dgrad64_kernel, and keeps four waves for the data gradients of a two-stream backward pass; the parity (fp32) mode and a region count
    other than 64 keep the generic launches."""
    kernels = lambda ops: [getattr(op, "meta", {}).get("kernel") for op in ops if getattr(op, "meta", None)]
    e = _dry_engine("bf16")
    inf = kernels(e.plan(64, False, False).fwd)
    assert "stem_conv_pool_kernel" in inf and "stem_conv_kernel" not in inf
    assert "head_conv_tail64_kernel<bf16,false>" in inf
    # r6: layer1's blocks are one launch each; EVERY stride-2 3x3 conv (the three stage entries WITH their 1x1 shortcuts, Patch-PnP's three) runs on
    # the parity-plane kernel -- 8-wide maps two images to a tile -- and the ConvTranspose's forward pass on the parity-class kernel; the generic
    # kernel keeps nothing of the forward pass (fc_r | fc_t: one launch with fc2's finish pass and the pose decode)
    assert sum(k == "block64_eval_kernel" for k in inf) == 3 and not any(k.startswith("conv3x3_halo_kernel<bf16,8,16,64") for k in inf)
    assert sum(k == "conv3x3s2_kernel<true>" for k in inf) == 3 and sum(k == "conv3x3s2_kernel<false>" for k in inf) == 3
    assert sum(k == "conv3x3s2_dgrad_kernel<false,false> (forward)" for k in inf) == 1
    assert sum(k.startswith("conv_gemm_kernel") for k in inf) == 0, [k for k in inf if k.startswith("conv_gemm")]   # (fc_r | fc_t ride in the pose kernel)
    assert sum(k.endswith(",2,1>") or k.endswith(",2>") for k in inf if k.startswith("conv3x3_halo_kernel")) == 18   # layer3 + layer4 + the 16x16 head conv: eight waves
    tr = e.plan(64, True, True)
    fwd, bwd = kernels(tr.fwd), kernels(tr.bwd)
    assert "stem_conv_kernel" in fwd and "stem_conv_pool_kernel" not in fwd            # train mode: bn1 needs the batch statistics first
    assert sum(k == "conv3x3s2_kernel<true>" for k in fwd) == 3 and sum(k == "conv3x3s2_kernel<false>" for k in fwd) == 3 and "block64_eval_kernel" not in fwd
    assert sum(k == "conv3x3s2_dgrad_kernel<false,false> (forward)" for k in fwd) == 1
    assert sum(k == "conv3x3s2_dgrad_kernel<true,true>" for k in bwd) == 3 and sum(k == "conv3x3s2_dgrad_kernel<false,false>" for k in bwd) == 3
    assert sum(k.startswith("conv_gemm_kernel") for k in bwd) == 2     # fc_rt / fc2 data gradients; fc1's: the split-K GEMM; the ConvTranspose's: the parity-plane kernel with the BatchNorm-backward epilogue
    assert sum(k == "conv3x3s2_kernel<false> (data gradient)" for k in bwd) == 1
    assert "head_conv_tail64_kernel<bf16,true>" in fwd and "head_out_dgrad64_kernel<bf16>" in bwd
    assert not any(k.startswith("conv3x3_halo_kernel") and k.split(",")[-1].rstrip(">") == "2" for k in bwd)   # four-wave data gradients (side stream on)
    assert any(k.startswith("conv3x3_halo_kernel") and k.split(",")[-1].rstrip(">") == "2" for k in fwd)
    e32 = _dry_engine("fp32")
    k32 = kernels(e32.plan(64, True, True).fwd + e32.plan(64, True, True).bwd)
    assert not any(k.startswith(("head_conv_tail", "head_out_dgrad", "stem_conv")) for k in k32)


def test_round6_plan_logic_on_dry_plans():
    """r6 host logic, launch lists only: (1) the grouped weight gradient of a bucket takes no more k-steps per workgroup than its large shape classes
    have (layer4 + layer3: 1088 equal workgroups; the head's ConvTranspose, 1 % of its bucket, does not set the length: 768 stays); (2) small
    side-stream ops wait for the end of their bucket: six switches from the main stream to the side stream per backward pass, and every deferred
    op sits in front of its bucket's grouped launch; (3) the two launches that build dL/dfc are marked as skippable for a seeded forward pass."""
    e = _dry_engine("bf16")
    tr = e.plan(64, True, True)
    grouped = [op.meta["layer"] for op in tr.bwd if getattr(op, "meta", None) and "wgrad_multi" in op.meta.get("kernel", "")]
    assert [g.split("(")[1] for g in grouped] == ["168 wg)", "768 wg)", "1088 wg)", "756 wg)"], grouped   # (Patch-PnP bucket: at least 64 k-steps per workgroup)
    side = [bool(getattr(op, "side", False)) for op in tr.bwd]
    forks = sum(1 for i in range(1, len(side)) if side[i] and not side[i - 1])
    assert forks == 6, forks
    marks = sorted(tr._bucket_marks())
    lo = 0
    for end in marks:      # per bucket: every deferred op in front of the bucket's grouped launch
        seg = tr.bwd[lo:end + 1]
        gl = [i for i, op in enumerate(seg) if getattr(op, "meta", None) and "wgrad_multi" in op.meta.get("kernel", "")]
        de = [i for i, op in enumerate(seg) if getattr(op, "defer", False)]
        assert len(gl) == 1 and all(i < gl[0] for i in de), (lo, end, gl, de)
        lo = end + 1
    assert sum(1 for op in tr.bwd if getattr(op, "defer", False)) == 7      # fc_rt / fc2 / fc1 weight gradients, two fc bias gradients, two 1x1 shortcut weight gradients
    assert sum(1 for op in tr.bwd if getattr(op, "seed", False)) == 2       # combine3 + cast: skipped when gdrn_pose_loss wrote dL/dfc itself
    # inference plans have no backward pass and no loss rows
    inf = e.plan(64, False, False)
    assert not inf.bwd and not any(getattr(op, "seed", False) for op in inf.fwd)
