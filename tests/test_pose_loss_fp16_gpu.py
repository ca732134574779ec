"""The format-dependent cases of tests/test_pose_loss_gpu.py a second time on libgdrn_hip_f16.so (the same kernel source built with IEEE half as
the 16-bit format): the module source is executed again with `BF16` bound to the fp16 dtype code, so dfc_comb, f2_out and w_rt are fp16 and the
replays round to fp16.  The decode, the losses and the fp32 gradient planes do not depend on the format: one generic case stands for them."""
import importlib.util
import os

from gdrnet_amd import cabi

_src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_pose_loss_gpu.py")
_spec = importlib.util.spec_from_file_location("_test_pose_loss_fp16_impl", _src)
_mod = importlib.util.module_from_spec(_spec)
_mod.__dict__["__HALF__"] = cabi.F16
_spec.loader.exec_module(_mod)
assert _mod.IS_F16 and _mod.KIND == "fp16" and len(_mod.GENERIC) == 1

pytestmark = _mod.pytestmark
H = _mod.H   # the module-scoped fixture (loads the fp16 library)
test_generic_every_output = _mod.test_generic_every_output
test_dfc_comb_is_the_weighted_sum_at_the_storage_width = _mod.test_dfc_comb_is_the_weighted_sum_at_the_storage_width
test_fc_tail_in_the_same_launch = _mod.test_fc_tail_in_the_same_launch
