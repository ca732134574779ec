// Device helpers of the head tail (head_tail.hip) and of the fused 1x1 output conv + tail (head_conv.hip): the 16-lanes-per-pixel lane map, ONE
// copy of the 64-region per-pixel body and of the loss-sum epilogue.
#pragma once
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "common.h"

// 16 lanes per pixel (one DPP row), 4 pixels per wave: lane q holds classes q, q+16, ... -- contiguous 64-byte loads,
// row reductions in 4 DPP adds.  (The first version used one wave per pixel with 6-step cross-lane reductions and ran
// at ~0.5 TB/s.)
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true)));
    return v;
}

template <typename T> __device__ __forceinline__ void store4(T* p, const float (&v)[4]);
template <> __device__ __forceinline__ void store4<float>(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t* p, const float (&v)[4]) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
}
template <typename T> __device__ __forceinline__ void load4(const T* p, float (&v)[4]);
template <> __device__ __forceinline__ void load4<float>(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <> __device__ __forceinline__ void load4<bf16_t>(const bf16_t* p, float (&v)[4]) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = h16lo(t.x); v[1] = h16hi(t.x);
    v[2] = h16lo(t.y); v[3] = h16hi(t.y);
}

// ------------------------------------------------------------------------------------------ one pixel of the 64-region tail
// The shape the network uses (64 regions, 72-float head rows): lane q of a pixel's 16 lanes holds the FOUR consecutive classes 4q..4q+3
// (r = the logits at float 4 + 4q; class 64 = h68 rides on lane 15), h03 = mask, x, y, z.  The callers load; nothing here touches the logits' memory.
// tail64_store: softmax over classes 1..64 (region[:, 1:]) as one 4-channel store per lane into pixel m's pnp row (72 channels), with the 2-D
// coordinates (c2x, c2y) and the extent-scaled xyz (GDRN.py:156-169).  Returns the row, pnp + m * pcs, which is formed BEHIND the softmax: handed in
// ready-made the compiler issued the pixel's loads in another order and the 16-bit eval kernel took 26.9 instead of 26.1 us (tools/htbench.py).
template <typename T>
__device__ __forceinline__ T* tail64_store(T* pnp, long long m, int pcs, int q, const float (&r)[4], const float (&h03)[4], float h68, float c2x,
                                           float c2y, const float (&ex)[3]) {
    const float r64 = (q == 15) ? h68 : -INFINITY;
    float mx = fmaxf(fmaxf(q == 0 ? -INFINITY : r[0], r[1]), fmaxf(fmaxf(r[2], r[3]), r64));
    mx = row16_max(mx);
    float e[4], e64;
    e[0] = (q == 0) ? 0.f : expf(r[0] - mx);
#pragma unroll
    for (int j = 1; j < 4; ++j) e[j] = expf(r[j] - mx);
    e64 = (q == 15) ? expf(r64 - mx) : 0.f;
    const float inv = 1.f / row16_sum(e[0] + e[1] + e[2] + e[3] + e64);
    T* o = pnp + m * pcs;
    float v[4] = {e[0] * inv, e[1] * inv, e[2] * inv, e[3] * inv};
    if (q == 0) v[0] = c2y;                                        // channel 4 = second roi_coord_2d channel
    store4<T>(o + 4 + 4 * q, v);                                   // channels 4 + 4q .. 7 + 4q
    // (both rows are built in front of the branches: with each inside its branch the compiler merged the two fp32 stores into one block of four
    // one-float stores at selected offsets, 30.8 instead of 29.5 us for the fp32 eval kernel; the arithmetic still sinks into the branch)
    const float w15[4] = {e64 * inv, 0.f, 0.f, 0.f};               // channel 68 = class 64, 69..71 pad
    const float w14[4] = {(h03[1] - 0.5f) * ex[0], (h03[2] - 0.5f) * ex[1], (h03[3] - 0.5f) * ex[2], c2x};
    if (q == 15) store4<T>(o + 68, w15);
    else if (q == 14) store4<T>(o, w14);
    return o;
}

// tail64_loss: the pixel's cross entropy over the 65 classes of logits * visib (GDRN.py:392-400) and its masked L1 terms (GDRN.py:345-391), added
// to a[0..2] = xyz, a[3] = mask, a[4] = cross entropy, a[5] = visible pixels -- of lane q == 0 only
__device__ __forceinline__ void tail64_loss(float (&a)[6], int q, const float (&r)[4], const float (&h03)[4], float h68, float mv, float mt,
                                            long long gr, const float (&gx)[3]) {
    const int tgt = (int)(gr * (long long)mv);
    float z[4], zt = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        z[j] = r[j] * mv;
        if (4 * q + j == tgt) zt = z[j];
    }
    const float z64 = (q == 15) ? h68 * mv : -INFINITY;
    if (q == 15 && tgt == 64) zt = z64;
    float mz = fmaxf(fmaxf(z[0], z[1]), fmaxf(fmaxf(z[2], z[3]), z64));
    mz = row16_max(mz);
    float es = expf(z[0] - mz) + expf(z[1] - mz) + expf(z[2] - mz) + expf(z[3] - mz) + (q == 15 ? expf(z64 - mz) : 0.f);
    es = row16_sum(es);
    zt = row16_sum(zt);
    if (q == 0) {
        a[4] += (logf(es) + mz) - zt;
        a[5] += mv;
        a[3] += fabsf(h03[0] - mt);
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] += fabsf(h03[1 + c] * mv - gx[c] * mv);
    }
}

// ------------------------------------------------------------------------------------------ loss sums of a workgroup
// a[6] of lane q == 0 of each of the 16 pixel groups of a 256-thread workgroup -> six sums in double, added in a fixed order.  Holds a
// __syncthreads() and its own LDS: EVERY thread of the workgroup calls it exactly once, outside divergent control flow.
// acc_rows: this workgroup's partial row (summed in a fixed order by gdrn_map_loss_finalize_rows) instead of 6 atomics per
// workgroup onto one cache line: 24 k same-line atomics across 8 XCDs cost the kernel 15 us
__device__ __forceinline__ void loss_sums_store(const float (&a)[6], double* acc, bool acc_rows) {
    __shared__ float red[6][16];
    if ((threadIdx.x & 15) == 0)
#pragma unroll
        for (int k = 0; k < 6; ++k) red[k][threadIdx.x >> 4] = a[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) v += (double)red[threadIdx.x][i];
        if (acc_rows) acc[8 + (size_t)blockIdx.x * 8 + threadIdx.x] = v;
        else unsafeAtomicAdd(&acc[threadIdx.x], v);
    }
}
