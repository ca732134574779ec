"""tests/test_conv3x3_edges_gpu.py a second time on libgdrn_hip_f16.so (the same kernel source built with IEEE half as the 16-bit format): the
module source is executed again with `BF16` bound to the fp16 dtype code, so every operand and output is fp16, the references round to fp16
and the bounds carry fp16's unit roundoff and subnormal step.  The fp32 instantiation does not depend on the format and is left to the bf16
module."""
import importlib.util
import os

from gdrnet_amd import cabi

_src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_conv3x3_edges_gpu.py")
_spec = importlib.util.spec_from_file_location("_test_conv3x3_edges_fp16_impl", _src)
_mod = importlib.util.module_from_spec(_spec)
_mod.__dict__["__HALF__"] = cabi.F16
_spec.loader.exec_module(_mod)
assert _mod.IS_F16 and _mod.HALF == "fp16"

pytestmark = _mod.pytestmark
H = _mod.H   # the module-scoped fixture (loads the fp16 library)
test_forward_per_element_with_fences = _mod.test_forward_per_element_with_fences
test_data_gradient_per_element = _mod.test_data_gradient_per_element
test_fused_bn_backward_epilogue_per_element_and_row_by_row = _mod.test_fused_bn_backward_epilogue_per_element_and_row_by_row
test_operand_transform_and_the_conv_of_its_own_output = _mod.test_operand_transform_and_the_conv_of_its_own_output
test_block64_per_element = _mod.test_block64_per_element
test_refusals_by_return_code_with_the_output_untouched = _mod.test_refusals_by_return_code_with_the_output_untouched
test_patch_offsets_past_32_bits_are_refused = _mod.test_patch_offsets_past_32_bits_are_refused
