"""tests/test_norm_edges_gpu.py a second time on libgdrn_hip_f16.so (the same kernel sources built with IEEE half as the 16-bit format): the
module source is executed again with `BF16` bound to the fp16 dtype code, so operands are stored as fp16, the bounds take u = 2^-11 and the cast
tests walk the fp16 patterns.  The fp32 instantiations and the exact launch-geometry regime (one storage type per case) are not repeated."""
import importlib.util
import os

from gdrnet_amd import cabi

_src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_norm_edges_gpu.py")
_spec = importlib.util.spec_from_file_location("_test_norm_edges_fp16_impl", _src)
_mod = importlib.util.module_from_spec(_spec)
_mod.__dict__["__HALF__"] = cabi.F16
_spec.loader.exec_module(_mod)
assert _mod.IS_F16 and _mod.DTS == [cabi.F16]

pytestmark = _mod.pytestmark
H = _mod.H   # the module-scoped fixture (loads the fp16 library)
for _k, _v in list(vars(_mod).items()):
    if _k.startswith("test_"):
        globals()[_k] = _v
