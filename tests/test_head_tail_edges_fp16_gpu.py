"""The format-dependent cases of tests/test_head_tail_edges_gpu.py a second time on libgdrn_hip_f16.so (the same kernel source built with IEEE
half as the 16-bit format): the module source is executed again with `BF16` bound to the fp16 dtype code, so pnp, d_pnp, d_head and the fused
kernels' operands are fp16 and the references round to fp16.  The fp32 cases do not depend on the format and are left to the bf16 module; the
generic kernels run at two region counts."""
import importlib.util
import os

from gdrnet_amd import cabi

_src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_head_tail_edges_gpu.py")
_spec = importlib.util.spec_from_file_location("_test_head_tail_edges_fp16_impl", _src)
_mod = importlib.util.module_from_spec(_spec)
_mod.__dict__["__HALF__"] = cabi.F16
_spec.loader.exec_module(_mod)
assert _mod.IS_F16 and _mod.KIND == "fp16" and _mod.DTS == [cabi.F16]

pytestmark = _mod.pytestmark
H = _mod.H   # the module-scoped fixture (loads the fp16 library)
test_fast_path_every_output_per_element = _mod.test_fast_path_every_output_per_element
test_generic_path_every_output_per_element = _mod.test_generic_path_every_output_per_element
test_fused_conv_tail_per_element = _mod.test_fused_conv_tail_per_element
test_fused_out_dgrad_per_element = _mod.test_fused_out_dgrad_per_element
test_fused_kernels_refuse_what_they_cannot_run = _mod.test_fused_kernels_refuse_what_they_cannot_run
test_short_rows_are_refused_with_every_output_untouched = _mod.test_short_rows_are_refused_with_every_output_untouched
