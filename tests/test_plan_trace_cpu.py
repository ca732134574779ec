"""CPU tests (-m "not gpu") of the launch lists through tools/plan_trace.py: a dry plan's ops are called against a recording stand-in of the
library, so every launch argument of every op is seen without a GPU.  No golden trace is kept here: a change of plan.py is checked by
diffing the tool's output of the commit before against the commit after (tools/README.md)."""
import importlib.util
import os
import re

import pytest

from gdrnet_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("plan_trace", os.path.join(ROOT, "tools", "plan_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PT = _tool()


@pytest.fixture(scope="module")
def train():
    return PT.trace("bf16", 4, True, True)


@pytest.fixture(scope="module")
def infer():
    return PT.trace("bf16", 4, False, False)


def test_every_op_of_a_train_plan_launches(train):
    """(a) each op of fwd and bwd makes at least one library call when it is called (none raised: the fixture came back), and each call
    is one line of the trace"""
    lists = {nm for nm, _, _ in train.ops}
    assert lists == {"fwd", "bwd"}, lists   # (a train plan has no eval-mode preparation)
    silent = [(nm, i) for nm, i, names in train.ops if not names]
    assert not silent, silent
    assert sum(len(names) for _, _, names in train.ops) == len(train.names)
    assert sum(1 for ln in train.text.splitlines() if ln.startswith("gdrn_")) == len(train.names)


def test_two_fresh_engines_trace_identically(train):
    """(b) the text names pointers by first appearance: what the host allocator returned does not show"""
    again = PT.trace("bf16", 4, True, True)
    assert again.text == train.text
    assert not re.search(r"0x[0-9a-f]{6,}|\b\d{14,}\b", train.text)   # no raw address anywhere (the largest number of a bs = 4 trace is a FLOP count < 1e12)


def test_inference_plan_launches_no_backward_kernel(infer):
    """(c) eval BatchNorm, no losses: no call of an entry point whose name contains bwd, wgrad or dgrad, neither in the forward list nor in
    the eval-mode preparation.  One entry point carries such a name in a forward role: the head's ConvTranspose2d runs its FORWARD pass on
    gdrn_conv3x3s2_dgrad (the same sum as a stride-2 conv's data gradient, Plan._convT_fwd).  That call is told from a data gradient by its
    arguments -- the forward epilogue (folded BatchNorm shift as bias, ReLU), which no data-gradient launch sets -- and is allowed exactly once."""
    assert {nm for nm, _, _ in infer.ops} == {"prep", "fwd"}
    lines = [ln for ln in infer.text.splitlines() if ln.startswith("gdrn_")]
    assert [ln.split()[0] for ln in lines] == infer.names
    bad = [ln for ln in lines if any(w in ln.split()[0] for w in ("bwd", "wgrad", "dgrad"))]
    convT = [ln for ln in bad if ln.startswith("gdrn_conv3x3s2_dgrad S2dParams(") and re.search(r",bias=p\d+,act=1\)", ln) and ",stats=0," in ln
             and ",dyd=0," in ln and ",bnb_x=0," in ln and ",Hi=16,Wi=16,Cin=256," in ln]
    assert len(convT) == 1 and bad == convT, bad
    hdr = infer.text.splitlines()[infer.text.splitlines().index(convT[0]) - 1]
    assert "(forward)" in hdr and "'layer': 'rot_head_net.features.0'" in hdr, hdr
    assert all(names for nm, _, names in infer.ops if nm == "fwd")
    assert "-- bucket_marks None" in infer.text and "-- grad_group {}" in infer.text


def test_queries_that_pass_through_take_no_stream():
    """the tool lets an entry point reach the real library by the end of its name: those are exactly host-only (include/gdrn_hip.h: no stream
    parameter), and every entry point that takes a stream is recorded"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdrn_hip.h")).read(), flags=re.S)
    decl = dict(re.findall(r"\b(?:int|long long)\s+(gdrn_[a-z0-9_]+)\s*\(([^)]*)\)", txt))
    assert set(decl) >= set(cabi._SIGS) - {"gdrn_half_format"} and len(decl) >= 100
    for name in cabi._SIGS:
        if PT.is_query(name):
            assert "stream" not in decl.get(name, ""), name
    launches = [n for n, args in decl.items() if "stream" in args]
    assert len(launches) >= 80 and not [n for n in launches if PT.is_query(n)]
    assert all(PT.QUERY.search(n) and "stream" in decl[n] for n in PT.LAUNCHES)


def test_configurations_cover_every_engine_switch():
    """the grid the tool writes: 3 dtypes x 4 batch sizes x 4 modes, and one variant per environment switch that changes a launch list"""
    names = [c[0] for c in PT.CONFIGS]
    assert len(names) == len(set(names)) == 48 + 11 + 2
    varied = {k for c in PT.CONFIGS for k in c[5]}
    from gdrnet_amd import switches

    src = open(os.path.join(ROOT, "gdr-net_amd", "engine.py")).read()
    read = set(re.findall(r'\bread\("(GDRN_[A-Z0-9_]+)"', src))   # what the engine reads is what the table says it reads
    assert read == {s.name for s in switches.TABLE.values() if s.read_at == switches.ENGINE} and len(read) == 11
    assert read - varied == {"GDRN_MAX_PLANS", "GDRN_LOSS_SCALE"}, read - varied   # (plan cache size, fp16 loss scale: no launch list depends on them)
