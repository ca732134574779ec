// Host side of the conv launches: what more than one conv source needs in front of a launch.  No device code, nothing exported.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/gdrn_hip.h"

// second-generation halo kernel (conv3x3_v3.hip), reached through the entry points of conv3x3_halo.hip with p->w_frag == 2
int gdrn_v3_config(const gdrn_conv_params* p);
int gdrn_v3_preferred(const gdrn_conv_params* p);
int gdrn_v3_tile(const gdrn_conv_params* p, int* th, int* tw, int* bn);
int gdrn_v3_launch(const gdrn_conv_params* p, void* stream);

// Raises the dynamic-LDS limit of one kernel (instantiation) to `bytes`, once per process and safe between host threads making their first
// launch together; the outcome of that one call is what every later call returns (a failed attribute call is not tried again).
template <auto Kernel>
bool lds_limit_once(size_t bytes) {
    static std::once_flag once;
    static bool ok = false;
    std::call_once(once, [bytes] {
        ok = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
    });
    return ok;
}

// The kernels form byte offsets in 32 bits: does the product of the factors (elements x stride x bytes per element ...) end below 2^32?
template <class... F>
constexpr bool fits_u32(F... factors) {
    return (1ull * ... * (unsigned long long)factors) < (1ull << 32);
}

// ---- the rules the two stride-1 3x3 halo kernels share (gdrn_conv3x3_halo, gdrn_v3_launch); each entry point applies them in its own order

constexpr int XF_MAX_CIN = 512;   // channels of the operand-transform table

// images of the launch: M must be whole maps of Ho x Wo pixels; 0 otherwise
inline int halo_images(const gdrn_conv_params& p) {
    const int hw = p.Ho * p.Wo;
    return (p.M > 0 && p.M % hw == 0) ? p.M / hw : 0;
}

// fused BatchNorm-backward epilogue (p.bnb_x): fast epilogue only, whole channel tiles of bn; osz = the bytes per element that the entry point's
// 32-bit-offset limits on the epilogue's tensors are scaled by
inline int halo_bnb_rules(const gdrn_conv_params& p, int bn, int osz) {
    if (!p.bnb_x) return GDRN_OK;
    if (!p.bnb_mean || !p.bnb_invstd || !p.bnb_rows || (p.bnb_scale != nullptr) != (p.bnb_shift != nullptr)) return GDRN_ERR_ARG;
    if (p.bias || p.act || p.out_f32 || (p.Cout % bn) || (p.bnb_cs & 3) || p.bnb_cs < p.Cout) return GDRN_ERR_SHAPE;
    if (!fits_u32(p.M, p.bnb_cs, osz)) return GDRN_ERR_SHAPE;
    return GDRN_OK;
}

// operand transform while staging (p.xf_mode)
inline int halo_xf_rules(const gdrn_conv_params& p) {
    if (!p.xf_mode) return GDRN_OK;
    if (p.xf_mode < 0 || p.xf_mode > 4 || !p.xf_c || p.Cin > XF_MAX_CIN || (p.Cin & 7)) return GDRN_ERR_ARG;
    if (p.xf_mode >= 2 && !p.xf_x2) return GDRN_ERR_ARG;
    if (p.xf_mode == 4 && (!p.xf_msc || !p.xf_msh)) return GDRN_ERR_ARG;
    if (p.xf_mode != 2 && p.xf_c2) return GDRN_ERR_ARG;
    return GDRN_OK;
}
