"""tests/test_wgrad_edges_gpu.py a second time on libgdrn_hip_f16.so (the same kernel source built with IEEE half as the 16-bit format): the
module source is executed again with `BF16` bound to the fp16 dtype code, so every operand is fp16 and the references are built from fp16
values.  The generic kernel's fp32 instantiation does not depend on the format and is left to the bf16 module."""
import importlib.util
import os

from gdrnet_amd import cabi

_src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_wgrad_edges_gpu.py")
_spec = importlib.util.spec_from_file_location("_test_wgrad_edges_fp16_impl", _src)
_mod = importlib.util.module_from_spec(_spec)
_mod.__dict__["__HALF__"] = cabi.F16
_spec.loader.exec_module(_mod)
assert _mod.IS_F16 and _mod.HALF == "fp16"

pytestmark = _mod.pytestmark
H = _mod.H   # the module-scoped fixture (loads the fp16 library)
test_halo_every_split_request_slab_by_slab_reduced_and_with_atomics = _mod.test_halo_every_split_request_slab_by_slab_reduced_and_with_atomics
test_halo_exact_operands_bit_for_bit_past_eight_splits = _mod.test_halo_exact_operands_bit_for_bit_past_eight_splits
test_reduce_hand_filled_slabs_exactly_with_skipped_slots_fenced = _mod.test_reduce_hand_filled_slabs_exactly_with_skipped_slots_fenced
test_grouped_launch_per_element_and_bit_for_bit_with_the_single_launch = _mod.test_grouped_launch_per_element_and_bit_for_bit_with_the_single_launch
test_generic_kernel_per_element_onto_a_filled_gradient = _mod.test_generic_kernel_per_element_onto_a_filled_gradient
test_generic_kernel_exact_operands_bit_for_bit_past_eight_splits = _mod.test_generic_kernel_exact_operands_bit_for_bit_past_eight_splits
test_halo_refusals_by_return_code_with_every_output_untouched = _mod.test_halo_refusals_by_return_code_with_every_output_untouched
test_generic_refusals_by_return_code_with_the_gradient_untouched = _mod.test_generic_refusals_by_return_code_with_the_gradient_untouched
test_halo_offsets_past_32_bits_are_refused = _mod.test_halo_offsets_past_32_bits_are_refused
