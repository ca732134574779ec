// What the fp64 evaluation kernels (pose_metrics.hip, bop_metrics.hip, sixd_scores.hip, render.hip, pnp.hip) share: the posed point and the fixed-order sums.
// Include after common.h.  render.hip and bop_metrics.hip switch floating-point contraction OFF behind their includes, the other two leave it on:
// everything here is explicit fma() and plain additions only, so it is the same operation sequence on both sides of that pragma.
#pragma once

namespace {

struct V3 { double x, y, z; };

__host__ __device__ __forceinline__ V3 load3(const double* p) { return V3{p[0], p[1], p[2]}; }

// R p + t.  Explicit fma chains: the same operations at every call site, whatever the compiler would contract -- a point posed on its way into
// LDS and the same point posed into a register are the same bits, so an estimate equal to the ground truth scores exactly 0, as in the reference.
__host__ __device__ __forceinline__ V3 xform(const double* R, const double* t, V3 p) {
    V3 o;
    o.x = fma(R[0], p.x, fma(R[1], p.y, fma(R[2], p.z, t[0])));
    o.y = fma(R[3], p.x, fma(R[4], p.y, fma(R[5], p.z, t[1])));
    o.z = fma(R[6], p.x, fma(R[7], p.y, fma(R[8], p.z, t[2])));
    return o;
}

__device__ __forceinline__ double wave_sum_f64(double v) {   // xor tree: a fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum for 256-thread blocks in a fixed order; result valid in every thread.  `red` is >= 4 doubles of LDS.
__device__ __forceinline__ double block_sum_256_f64(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// every entry of a host index vector within [0, bound): what each entry point checks before its first launch
inline int host_in_range(const int* host, int n, int bound) {
    for (int i = 0; i < n; ++i)
        if (host[i] < 0 || host[i] >= bound) return 0;
    return 1;
}

}  // namespace
